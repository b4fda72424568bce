"""rustray_amd/csrc/rr_scene_build.h (the checks, record makers, per-mesh trees and the top level behind rr_scene_create and the scene
edits) under AddressSanitizer + UBSan on the CPU: the padded world boxes never cull an item whose local box test the reference passes
(oracle: rro_item_box_hit), surface boxes lie inside the corner boxes and hold every vertex, each top-level tree names every item once
within its share of the traversal stack, the records of a small hand-made scene, every rejection of the shared checks, and the
texture pool's layout under appends."""
import os
import subprocess

from oracle import binding as ob
from tests.helpers import ROOT


def test_scene_build_under_asan(tmp_path):
    exe = str(tmp_path / "scene_build_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    oracle_dir = os.path.dirname(ob.build())
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe,
           os.path.join(ROOT, "tests", "native", "scene_build_test.cpp"), os.path.join(ROOT, "rustray_amd", "csrc", "rr_bvh.cpp"),
           "-L" + oracle_dir, "-loracle", "-Wl,-rpath," + oracle_dir]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "scene build test OK" in out.stdout, out.stdout + out.stderr
