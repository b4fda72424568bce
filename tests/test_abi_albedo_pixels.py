"""rr_albedo_pixels without a GPU: the yardstick of its sum on hand-made terms (rustray_amd/albedo.py), the header still compiles as C99
with the two declarations, both symbols are exported, bound and guarded, and every refusal that precedes the scene comes back with its
message, on a fake handle (tests/native/albedo_pixels_c99.c makes the same calls from C)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.albedo import mean_albedo
from rustray_amd.flat import make_config, rr_camera
from tests.helpers import ROOT, host_api_source

NAMES = ("rr_albedo_pixels", "rr_albedo_pixels_device")
F = np.float32


# ---- the yardstick
def test_mean_albedo_exact_thirds():
    # three terms of 1/3 (binary32, 11184811 * 2^-25): each is the tie 5592405.5 at scale 2^24 and rounds to the even 5592406 by itself;
    # the sum is 16777218 = 1 + 2^-23, not the 1 a float sum would give
    third = F(1.0) / F(3.0)
    a = np.full((1, 3, 3), third, F)
    a[0, :, 1] = [0.0, 1.0, 0.5]             # 0 + 2^24 + 2^23 over 3
    a[0, :, 2] = [1.0, 1.0, 1.0]
    out = mean_albedo(a, 3)
    assert out.dtype == np.float32 and out.shape == (1, 3)
    assert float(third) * 2.0 ** 24 == 5592405.5
    assert out[0, 0] == F(F(16777218.0 * 2.0 ** -24) / F(3.0)) and out[0, 0] != F(F(1.0) / F(3.0))
    assert out[0, 1] == F(F(1.5) / F(3.0)) and out[0, 2] == F(1.0)
    # a term is rounded by itself, to nearest-even: 2^-25 is a tie and goes to 0, 3 * 2^-25 to 2 * 2^-24
    t = np.zeros((2, 2, 3), F)
    t[0, :, 0] = [2.0 ** -25, 2.0 ** -25]
    t[1, :, 0] = [3 * 2.0 ** -25, 3 * 2.0 ** -25]
    out = mean_albedo(t, 2)
    assert out[0, 0] == 0.0 and out[1, 0] == F(F(4 * 2.0 ** -24) / F(2.0))


def test_mean_albedo_clamp():
    a = np.zeros((2, 2, 3), F)
    a[0, :, 0] = [40000.0, 1.0]              # above the colour clamp of 32768: it adds the clamp
    a[1, :, 0] = [-1.0e9, 0.25]
    out = mean_albedo(a, 2)
    assert out[0, 0] == F(F(32769.0) / F(2.0)) and out[1, 0] == F(F(-32768.0 + 0.25) / F(2.0))
    assert (out[:, 1:] == 0.0).all()


def test_mean_albedo_nonfinite_terms():
    a = np.full((5, 4, 3), 0.5, F)
    a[0, 1, 0] = np.nan
    a[1, 2, 1] = np.inf
    a[2, 0, 2] = -np.inf
    a[3, 0, 0], a[3, 3, 0] = np.inf, -np.inf
    a[4, 0, 1], a[4, 1, 1] = np.nan, np.inf
    out = mean_albedo(a, 4)
    assert np.isnan(out[0, 0]) and out[0, 1] == 0.5 and out[0, 2] == 0.5     # a flag poisons its own channel only
    assert out[1, 1] == np.inf and out[1, 0] == 0.5
    assert out[2, 2] == -np.inf and out[2, 1] == 0.5
    assert np.isnan(out[3, 0]) and out[3, 1] == 0.5                          # +inf and -inf in one pixel and channel
    assert np.isnan(out[4, 1])                                               # NaN wins over +inf


def test_mean_albedo_all_misses_and_shapes():
    out = mean_albedo(np.zeros((7, 8, 3), F), 8)
    assert out.shape == (7, 3) and (out == 0.0).all() and not np.signbit(out).any()
    assert mean_albedo(np.zeros((0, 4, 3), F), 4).shape == (0, 3)
    with pytest.raises(ValueError):
        mean_albedo(np.zeros((2, 4, 3), F), 8)
    with pytest.raises(ValueError):
        mean_albedo(np.zeros((2, 4), F), 4)


# ---- the ABI
def test_c99_host(tmp_path):
    exe = str(tmp_path / "albedo_pixels_c99")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "albedo_pixels_c99.c"),
                           "-L" + libdir, "-lrustray_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "albedo pixels c99 OK" in out.stdout, out.stdout + out.stderr


def test_exported_bound_and_guarded():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    src = host_api_source()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None
        assert re.search(r"\bint " + n + r"\(rr_scene\* scene, const rr_camera\* camera, const rr_config\* config, const uint16_t\* sample_xy", header)
        assert re.search(r"\bint " + n + r"\([^{]*\) try \{", src), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
    assert "rr_api_albedo_pixels.h" in capi.LIB_SOURCES
    assert len(L.rr_albedo_pixels.argtypes) == 8 and len(L.rr_albedo_pixels_device.argtypes) == 9
    assert "#define RR_ABI_VERSION 3u" in header
    assert "rr_albedo_pixels and rr_albedo_pixels_device came after those" in header


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
    cfg = make_config(samples=4)
    alb = np.full(6 * 12, 0x5a, np.uint8)
    p_alb = C.c_void_p(alb.ctypes.data)
    fake = C.c_void_p(alb.ctypes.data)       # never dereferenced: every call below is refused by its arguments alone
    xy = np.array([0, 1 | (1 << 16)], np.uint32)
    p_xy = C.c_void_p(xy.ctypes.data)
    err = lambda: L.rr_last_error()
    for fn in (lambda *a: L.rr_albedo_pixels(*a, None), lambda *a: L.rr_albedo_pixels_device(*a, None, None)):
        # 1. a NULL scene, camera or config, whatever else is wrong with the call
        assert fn(None, C.byref(cam), C.byref(cfg), None, None, 5, None) == -1 and b"NULL argument" in err()
        assert fn(fake, None, C.byref(cfg), None, None, 5, None) == -1 and b"NULL argument" in err()
        assert fn(fake, C.byref(cam), None, None, None, 5, None) == -1 and b"NULL argument" in err()
        # 2. the whole config and the camera, as every frame call checks them
        bad_cfg = make_config(samples=0)
        assert fn(fake, C.byref(cam), C.byref(bad_cfg), None, None, 6, p_alb) == -1 and b"samples must be >= 1" in err()
        deep = make_config(samples=4, max_recursion=1000)      # ignored by the call, checked all the same
        assert fn(fake, C.byref(cam), C.byref(deep), None, None, 6, p_alb) == -2 and b"max_recursion" in err()
        for w, h in ((0, 2), (3, 0), (65536, 2), (3, 65536)):
            bad = _camera(w, h)
            assert fn(fake, C.byref(bad), C.byref(cfg), None, None, 0, p_alb) == -1 and b"bad frame size" in err()
        nan = _camera()
        nan.view_inverse[3] = float("nan")
        assert fn(fake, C.byref(nan), C.byref(cfg), None, None, 0, p_alb) == -1 and b"non-finite camera matrix" in err()
        # 3. the output, before n_pixels is looked at
        assert fn(fake, C.byref(cam), C.byref(cfg), None, None, 5, None) == -1 and b"albedo_out is required" in err()
        assert fn(fake, C.byref(cam), C.byref(cfg), None, None, 0, None) == -1 and b"albedo_out is required" in err()
        # 4. the pixel limit, before n_pixels is compared with the frame
        assert fn(fake, C.byref(cam), C.byref(cfg), None, None, (1 << 30) + 1, p_alb) == -2
        assert fn(fake, C.byref(cam), C.byref(cfg), None, p_xy, (1 << 30) + 1, p_alb) == -2
        # 5. n_pixels == 0: RR_OK, nothing is touched
        assert fn(fake, C.byref(cam), C.byref(cfg), None, None, 0, p_alb) == 0
        assert fn(fake, C.byref(cam), C.byref(cfg), None, p_xy, 0, p_alb) == 0
        # 6. without a list n_pixels is width * height
        for n in (1, 5, 7):
            assert fn(fake, C.byref(cam), C.byref(cfg), None, None, n, p_alb) == -1 and (b"%d pixels without a list" % n) in err() and b"3x2" in err()
    # the device form: alignment by argument name, then overlap, all before the scene is looked at
    dev = lambda *a: L.rr_albedo_pixels_device(fake, C.byref(cam), C.byref(cfg), None, *a, None, None)
    assert dev(None, 6, C.c_void_p(0x400002)) == -1 and b"albedo_out_dev is not 4-byte aligned" in err()
    assert dev(C.c_void_p(0x600001), 2, C.c_void_p(0x400000)) == -1 and b"pixel_xy_dev is not 4-byte aligned" in err()
    assert dev(C.c_void_p(0x400004), 2, C.c_void_p(0x400000)) == -1 and b"albedo_out_dev overlaps pixel_xy_dev" in err()
    # the host form checks its list before the scene: the first entry outside the frame, by index
    xy[1] = 3
    assert L.rr_albedo_pixels(fake, C.byref(cam), C.byref(cfg), None, p_xy, 2, p_alb, None) == -1 and b"pixel_xy[1] = (3, 0) lies outside the frame of 3x2" in err()
    assert (alb == 0x5a).all()


def test_python_layer_refuses_an_unknown_albedo_mode():
    from rustray_amd import renderer
    with pytest.raises(ValueError):
        renderer._check_albedo_mode("centre")
    for ok in (False, True, "mean"):
        renderer._check_albedo_mode(ok)
    assert renderer._mean_mode("mean") and not renderer._mean_mode(True) and not renderer._mean_mode(False)
