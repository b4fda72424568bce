"""rustray_amd/csrc/rr_query_pointers.h (may the scene's device address a buffer handed to a device-buffer ray query?) under
AddressSanitizer + UBSan on the CPU: every memory kind, own and other device, with and without peer access."""
import os
import re
import subprocess

from tests.helpers import ROOT


def test_query_pointer_decision_under_asan(tmp_path):
    exe = str(tmp_path / "query_pointer_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "query_pointer_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "query pointer test OK" in out.stdout, out.stdout + out.stderr


def test_the_header_is_host_only():
    """The decision is tested without a GPU because it needs none: the header includes nothing and calls no HIP function."""
    src = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_query_pointers.h")).read()
    assert "#include" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
