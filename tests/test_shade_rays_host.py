"""rr_shade_rays without a device: the symbol, the layout of rr_radiance (ctypes, the header's text, a C99 compile of the header)
and the argument checks that come before anything touches the scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_radiance
from tests.helpers import ROOT

HEADER = os.path.join(ROOT, "include", "rustray_hip.h")


def test_symbol_is_exported_and_bound():
    assert "rr_shade_rays" in capi.EXPORTS
    assert hasattr(C.CDLL(capi.LIB_PATH), "rr_shade_rays")
    assert hasattr(capi.DeviceScene, "shade_rays")


def test_record_is_thirty_two_bytes_and_matches_the_header():
    assert C.sizeof(rr_radiance) == 32
    assert [(rr_radiance.color.offset, rr_radiance.depth.offset, rr_radiance.normal.offset, rr_radiance.object_id.offset)] == [(0, 12, 16, 28)]
    body = re.search(r"typedef struct rr_radiance \{(.*?)\} rr_radiance;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in fields] == list(rr_radiance._fields_)


def test_record_in_a_c99_host(tmp_path):
    exe = str(tmp_path / "radiance_c99")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "radiance_c99.c"),
                           "-L" + libdir, "-lrustray_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "radiance c99 OK" in out.stdout, out.stdout + out.stderr


def test_argument_checks_that_need_no_device():
    L = capi.lib()
    cfg = make_config(samples=1, max_recursion=4)
    o = np.zeros((2, 3), np.float32); d = np.ones((2, 3), np.float32)
    out = (rr_radiance * 2)()
    op, dp = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    never_read = C.create_string_buffer(64)   # stands for a scene: every check below returns before the handle is looked at
    scene = C.cast(never_read, C.c_void_p)
    assert L.rr_shade_rays(None, C.byref(cfg), op, dp, 2, 1, None, out, None) == -1
    assert b"NULL" in L.rr_last_error()
    assert L.rr_shade_rays(None, C.byref(cfg), None, None, 0, 1, None, None, None) == -1      # a NULL scene, even for no results
    assert L.rr_shade_rays(scene, None, op, dp, 2, 1, None, out, None) == -1
    assert L.rr_shade_rays(scene, C.byref(cfg), op, dp, 2, 0, None, out, None) == -1           # rays_per_result 0
    assert b"rays_per_result" in L.rr_last_error()
    assert L.rr_shade_rays(scene, C.byref(cfg), op, dp, 2, 32767, None, out, None) == -2       # beyond RR_MAX_SAMPLES_WITH_TABLE
    assert b"rays_per_result" in L.rr_last_error()
    assert L.rr_shade_rays(scene, C.byref(cfg), None, None, 0, 1, None, None, None) == 0       # n_results == 0 touches nothing
    assert L.rr_shade_rays(scene, C.byref(cfg), op, dp, 0x7fffff01, 1, None, out, None) == -2  # refused before an array is read
    assert L.rr_shade_rays(scene, C.byref(cfg), None, dp, 2, 1, None, out, None) == -1
    assert L.rr_shade_rays(scene, C.byref(cfg), op, None, 2, 1, None, out, None) == -1
    assert L.rr_shade_rays(scene, C.byref(cfg), op, dp, 2, 1, None, None, None) == -1
    deep = make_config(samples=1, max_recursion=31)
    assert L.rr_shade_rays(scene, C.byref(deep), op, dp, 2, 1, None, out, None) == -2
    assert b"max_recursion" in L.rr_last_error()
