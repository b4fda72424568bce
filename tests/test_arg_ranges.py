"""rustray_amd/csrc/rr_arg_ranges.h (do the buffers handed to one record call overlap where they must not?) under AddressSanitizer +
UBSan on the CPU: every pair of small ranges against a byte-set model, in every role, and the named edge cases of the rule."""
import os
import re
import subprocess

from tests.helpers import ROOT


def test_arg_range_conflicts_under_asan(tmp_path):
    exe = str(tmp_path / "arg_ranges_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "arg_ranges_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "arg ranges test OK" in out.stdout, out.stdout + out.stderr


def test_the_header_is_host_only():
    """The rule is tested without a GPU because it needs none: the header includes nothing and calls no HIP function."""
    src = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_arg_ranges.h")).read()
    assert "#include" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
