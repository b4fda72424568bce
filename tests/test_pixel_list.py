"""rustray_amd/csrc/rr_pixel_list.h (the pixel list of rr_render_pixels: which entry lies outside the frame, where is a pixel's centre)
under AddressSanitizer + UBSan on the CPU, and what rr_render_pixels / rr_render_pixels_device refuse before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_camera, rr_radiance
from tests.helpers import ROOT, host_api_source


def test_pixel_list_under_asan(tmp_path):
    exe = str(tmp_path / "pixel_list_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "pixel_list_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pixel list test OK" in out.stdout, out.stdout + out.stderr


def test_the_header_is_host_only():
    """The list check is tested without a GPU because it needs none: the header includes nothing and calls no HIP function."""
    src = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_pixel_list.h")).read()
    assert "#include" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
    # and primary_slot_centres forms a region's centres through it: one expression for both kinds of slot
    setup = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_primary_setup.h")).read()
    assert '#include "rr_pixel_list.h"' in setup and "pixel_centre(slot_xy[j]" in setup


def _camera(w=50, h=38):
    cam = rr_camera()
    cam.width, cam.height = w, h
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    for i in range(16):
        cam.projection_inverse[i] = float(eye[i]); cam.view_inverse[i] = float(eye[i])
    return cam


def test_null_arguments_are_refused_without_a_device():
    """scene, camera, config and out are required by both forms; the refusal comes before the scene is looked at, so a made-up
    handle is never dereferenced and no device is needed."""
    L = capi.lib()
    cam, cfg = _camera(), make_config(samples=3)
    out = (rr_radiance * 4)()
    C.memset(out, 0x5a, C.sizeof(out))
    xy = np.arange(4, dtype=np.uint32)
    xy_p, out_p = xy.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p)
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused on its arguments alone
    for scene, cam_p, cfg_p, o in ((None, C.byref(cam), C.byref(cfg), out_p), (fake, None, C.byref(cfg), out_p), (fake, C.byref(cam), None, out_p),
                                   (fake, C.byref(cam), C.byref(cfg), None)):
        assert L.rr_render_pixels(scene, cam_p, cfg_p, None, xy_p, 4, o, None, None) == -1
        assert L.rr_last_error()
        assert L.rr_render_pixels_device(scene, cam_p, cfg_p, None, xy_p, 4, o, None, None, None) == -1
        assert L.rr_last_error()
    # the frame's own argument checks come first as well: the sample count, the recursion depth, the frame size
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(make_config(samples=0)), None, xy_p, 4, out_p, None, None) == -1
    assert b"samples" in L.rr_last_error()
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(make_config(samples=3, max_recursion=31)), None, xy_p, 4, out_p, None, None) == -2
    assert b"max_recursion" in L.rr_last_error()
    assert L.rr_render_pixels(fake, C.byref(_camera(0, 38)), C.byref(cfg), None, xy_p, 4, out_p, None, None) == -1
    # more than 2^30 pixels: refused before anything is allocated; no pixels at all: nothing to do
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(cfg), None, xy_p, (1 << 30) + 1, out_p, None, None) == -2
    assert L.rr_render_pixels_device(fake, C.byref(cam), C.byref(cfg), None, xy_p, (1 << 30) + 1, out_p, None, None, None) == -2
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(cfg), None, None, 0, out_p, None, None) == 0
    assert L.rr_render_pixels_device(fake, C.byref(cam), C.byref(cfg), None, None, 0, out_p, None, None, None) == 0
    # the whole frame is width * height pixels, and a host list is checked before the scene is locked: the first bad index is named
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(cfg), None, None, 50 * 38 - 1, out_p, None, None) == -1
    assert b"1899" in L.rr_last_error()
    bad = np.array([0, 49 | (37 << 16), 50, 5 | (38 << 16)], np.uint32)
    assert L.rr_render_pixels(fake, C.byref(cam), C.byref(cfg), None, bad.ctypes.data_as(C.c_void_p), 4, out_p, None, None) == -1
    assert b"pixel_xy[2]" in L.rr_last_error()
    # the device form's alignment rules
    assert L.rr_render_pixels_device(fake, C.byref(cam), C.byref(cfg), None, xy_p, 4, C.c_void_p(C.addressof(out) + 8), None, None, None) == -1
    assert b"aligned" in L.rr_last_error()
    assert bytes(out) == b"\x5a" * C.sizeof(out)


def test_pack_pixels():
    assert capi.pack_pixels([(3, 5), (49, 37)]).tolist() == [3 | (5 << 16), 49 | (37 << 16)]
    assert capi.pack_pixels(np.array([7, 1 << 16], np.uint32)).tolist() == [7, 65536]
    assert capi.pack_pixels(np.zeros((0, 2), np.int64)).shape == (0,)


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in ("rr_render_pixels", "rr_render_pixels_device"):
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
    # they sit in one extern "C" block, and nothing else does: every definition in it is one of the two
    block = src[src.index('extern "C" {\n'):]
    block = block[:block.index('} // extern "C"')]
    assert src.count('extern "C" {\n') == 1 and re.findall(r"^int (rr_[a-z_]+)\(", block, re.M) == ["rr_render_pixels_device", "rr_render_pixels"]
    assert "rr_pixel_list.h" in capi.LIB_SOURCES
