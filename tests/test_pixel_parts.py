"""rr_render_pixel_parts without a GPU: the (slot, sample) mapping of its primary rays (rustray_amd/csrc/rr_primary_setup.h) under
AddressSanitizer + UBSan on the CPU, and what rr_render_pixel_parts / rr_render_pixel_parts_device refuse before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_camera, rr_radiance
from tests.helpers import ROOT, host_api_source


def test_pixel_parts_mapping_under_asan(tmp_path):
    exe = str(tmp_path / "pixel_parts_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "pixel_parts_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "pixel parts test OK" in out.stdout, out.stdout + out.stderr


def _camera(w=50, h=38):
    cam = rr_camera()
    cam.width, cam.height = w, h
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    for i in range(16):
        cam.projection_inverse[i] = float(eye[i]); cam.view_inverse[i] = float(eye[i])
    return cam


def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    cam = _camera()
    cfg = make_config(samples=8)
    out = (rr_radiance * 4)()
    parts = (rr_radiance * (4 * 64))()
    C.memset(out, 0x5a, C.sizeof(out)); C.memset(parts, 0x5a, C.sizeof(parts))
    xy = np.arange(4, dtype=np.uint32)
    xy_p, out_p, parts_p = xy.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p), C.cast(parts, C.c_void_p)
    fake = C.c_void_p(0x1000)

    def host(n_parts, n=4, o=out_p, p=parts_p, config=cfg, scene=fake, lst=xy_p):
        return L.rr_render_pixel_parts(scene, C.byref(cam), C.byref(config), None, lst, n, n_parts, o, p, None)

    def device(n_parts, n=4, o=out_p, p=parts_p, config=cfg, scene=fake, lst=xy_p):
        return L.rr_render_pixel_parts_device(scene, C.byref(cam), C.byref(config), None, lst, n, n_parts, o, p, None, None)

    for call in (host, device):
        for k in (0, 1, 3, 128):
            assert call(k) == -1
            assert b"power of two" in L.rr_last_error() and str(k).encode() in L.rr_last_error()
        assert call(16) == -1                                   # 16 does not divide 8
        assert b"divide" in L.rr_last_error()
        assert call(4, config=make_config(samples=6)) == -1     # nor 4 six
        assert b"divide" in L.rr_last_error()
        assert call(2, n=(1 << 29) + 1) == -2                   # more than 2^30 slots: refused before anything is allocated
        assert b"2^30" in L.rr_last_error()
        assert call(64, n=(1 << 24) + 1, config=make_config(samples=64)) == -2
        assert call(2, o=None) == -1
        assert b"out" in L.rr_last_error()
        assert call(2, p=None) == -1
        assert b"parts_out" in L.rr_last_error()
        assert call(2, scene=None) == -1
        assert call(2, n=0, lst=None) == 0                      # nothing to do
        assert call(2, n=50 * 38 - 1, lst=None) == -1           # the whole frame is width * height pixels
    # the device form's alignment rule holds for both outputs
    assert device(2, o=C.c_void_p(C.addressof(out) + 8)) == -1
    assert b"aligned" in L.rr_last_error()
    assert device(2, p=C.c_void_p(C.addressof(parts) + 8)) == -1
    assert b"aligned" in L.rr_last_error()
    # a host list is checked before the scene is locked: the first bad index is named
    bad = np.array([0, 49 | (37 << 16), 50, 5 | (38 << 16)], np.uint32)
    assert host(2, lst=bad.ctypes.data_as(C.c_void_p)) == -1
    assert b"pixel_xy[2]" in L.rr_last_error()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and bytes(parts) == b"\x5a" * C.sizeof(parts)


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in ("rr_render_pixel_parts", "rr_render_pixel_parts_device"):
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
        assert getattr(capi.lib(), n).argtypes is not None
    assert "rr_api_parts.h" in capi.LIB_SOURCES
    assert hasattr(capi.DeviceScene, "render_pixel_parts") and hasattr(capi.DeviceScene, "render_pixel_parts_device")
