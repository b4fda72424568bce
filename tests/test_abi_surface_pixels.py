"""rr_surface_pixels without a GPU: the header still compiles as C99 with the two declarations, both symbols are exported and bound, both
entry points are guarded, and every refusal that needs no device comes in the order include/rustray_hip.h states
(tests/native/surface_pixels_c99.c makes the same calls from C)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import rr_camera
from tests.helpers import ROOT, host_api_source

NAMES = ("rr_surface_pixels", "rr_surface_pixels_device")


def test_c99_host(tmp_path):
    exe = str(tmp_path / "surface_pixels_c99")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "surface_pixels_c99.c"),
                           "-L" + libdir, "-lrustray_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "surface pixels c99 OK" in out.stdout, out.stdout + out.stderr


def test_exported_bound_and_guarded():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    src = host_api_source()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None
        assert re.search(r"\bint " + n + r"\(rr_scene\* scene, const rr_camera\* camera,", header)
        assert re.search(r"\bint " + n + r"\([^{]*\) try \{", src), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
    assert "rr_api_surface_pixels.h" in capi.LIB_SOURCES and "rr_pixel_list.h" in capi.LIB_SOURCES
    assert len(L.rr_surface_pixels.argtypes) == 6 and len(L.rr_surface_pixels_device.argtypes) == 7


def _camera(w=3, h=2) -> rr_camera:
    cam = rr_camera()
    cam.width, cam.height = w, h
    for k in range(4):
        cam.projection_inverse[5 * k] = 1.0
        cam.view_inverse[5 * k] = 1.0
    return cam


def test_refusals_without_a_device_in_the_headers_order():
    L = capi.lib()
    cam = _camera()
    out = np.full(6 * 128, 0x5a, np.uint8)
    alb = np.full(6 * 12, 0x5a, np.uint8)
    p_out, p_alb = C.c_void_p(out.ctypes.data), C.c_void_p(alb.ctypes.data)
    fake = C.c_void_p(out.ctypes.data)       # never dereferenced: every call below is refused by its arguments alone
    xy = np.array([0, 1 | (1 << 16)], np.uint32)
    p_xy = C.c_void_p(xy.ctypes.data)
    err = lambda: L.rr_last_error()
    for fn in (lambda *a: L.rr_surface_pixels(*a), lambda *a: L.rr_surface_pixels_device(*a, None)):
        # 1. a NULL scene (or camera), whatever else is wrong with the call
        assert fn(None, C.byref(cam), None, 5, None, None) == -1 and b"NULL argument" in err()
        assert fn(fake, None, None, 5, None, None) == -1 and b"NULL argument" in err()
        # 2. both outputs NULL, before the camera and n_pixels are looked at
        bad = _camera(0, 2)
        assert fn(fake, C.byref(bad), None, 5, None, None) == -1 and b"both NULL" in err()
        assert fn(fake, C.byref(cam), None, 0, None, None) == -1 and b"both NULL" in err()
        # 3. the camera checks of rr_render_pixels
        for w, h in ((0, 2), (3, 0), (65536, 2), (3, 65536)):
            bad = _camera(w, h)
            assert fn(fake, C.byref(bad), None, 0, p_out, None) == -1 and b"bad frame size" in err()
        nan = _camera()
        nan.view_inverse[3] = float("nan")
        assert fn(fake, C.byref(nan), None, 0, p_out, None) == -1 and b"non-finite camera matrix" in err()
        # 4. the pixel limit, before n_pixels is compared with the frame
        assert fn(fake, C.byref(cam), None, 0x7fffff01, p_out, None) == -2
        assert fn(fake, C.byref(cam), p_xy, 0x7fffff01, None, p_alb) == -2
        # 5. n_pixels == 0: RR_OK, nothing is touched
        assert fn(fake, C.byref(cam), None, 0, p_out, p_alb) == 0
        assert fn(fake, C.byref(cam), p_xy, 0, None, p_alb) == 0
        # 6. without a list n_pixels is width * height
        for n in (1, 5, 7):
            assert fn(fake, C.byref(cam), None, n, p_out, p_alb) == -1 and (b"%d pixels without a list" % n) in err() and b"3x2" in err()
    # the device form: alignment by argument name, then overlap, all before the scene is looked at
    dev = lambda *a: L.rr_surface_pixels_device(fake, C.byref(cam), *a, None)
    assert dev(None, 6, C.c_void_p(0x200008), C.c_void_p(0x400000)) == -1 and b"out_dev is not 16-byte aligned" in err()
    assert dev(None, 6, C.c_void_p(0x200000), C.c_void_p(0x400002)) == -1 and b"albedo_out_dev is not 4-byte aligned" in err()
    assert dev(C.c_void_p(0x600001), 2, C.c_void_p(0x200000), None) == -1 and b"pixel_xy_dev is not 4-byte aligned" in err()
    assert dev(None, 6, C.c_void_p(0x200000), C.c_void_p(0x200000 + 6 * 128 - 4)) == -1 and b"albedo_out_dev overlaps out_dev" in err()
    assert dev(C.c_void_p(0x200000 + 128), 2, C.c_void_p(0x200000), None) == -1 and b"out_dev overlaps pixel_xy_dev" in err()
    assert dev(C.c_void_p(0x400004), 2, None, C.c_void_p(0x400000)) == -1 and b"albedo_out_dev overlaps pixel_xy_dev" in err()
    # the host form checks its list before the scene: the first entry outside the frame, by index
    xy[1] = 3
    assert L.rr_surface_pixels(fake, C.byref(cam), p_xy, 2, p_out, p_alb) == -1 and b"pixel_xy[1] = (3, 0) lies outside the frame of 3x2" in err()
    assert (out == 0x5a).all() and (alb == 0x5a).all()


def test_python_layer_refuses_a_call_without_outputs():
    import pytest
    ds = capi.DeviceScene.__new__(capi.DeviceScene)      # no handle: the check precedes the library
    with pytest.raises(ValueError):
        capi.DeviceScene.surface_pixels(ds, _camera(), records=False, albedo=False)
