"""Adaptive sampling on the device, without a GPU: the arithmetic the list kernels share with the host (rustray_amd/csrc/rr_adaptive.h)
under AddressSanitizer + UBSan on the CPU, and what rr_refine_list_device, rr_render_adaptive and rr_render_adaptive_device refuse before
they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_radiance
from tests.helpers import ROOT, host_api_source
from tests.test_pixel_parts import _camera

NEW = ("rr_refine_list_device", "rr_render_adaptive", "rr_render_adaptive_device")


def test_block_order_and_half_error_under_asan(tmp_path):
    exe = str(tmp_path / "adaptive_order_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "adaptive_order_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "adaptive order test OK" in out.stdout, out.stdout + out.stderr


def test_capacity():
    for w, h in ((1, 1), (8, 8), (9, 1), (20, 12), (50, 38), (1280, 720)):
        assert capi.refine_list_capacity(w, h) == (w * h + 63) // 64 * 64


def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    cam = _camera()
    n = 50 * 38
    cfg = make_config(samples=1)
    out = (rr_radiance * n)()
    C.memset(out, 0x5a, C.sizeof(out))
    out_p = C.cast(out, C.c_void_p)
    fake = C.c_void_p(0x1000)
    count = C.c_uint32(77)

    def host(base=6, top=16, thr=0.1, o=out_p, camera=cam, scene=fake):
        return L.rr_render_adaptive(scene, C.byref(camera), C.byref(cfg), base, top, thr, None, None, o, None, None, None, C.byref(count), None)

    def device(base=6, top=16, thr=0.1, o=out_p, camera=cam, scene=fake, samples=None, error=None, rgba=None):
        return L.rr_render_adaptive_device(scene, C.byref(camera), C.byref(cfg), base, top, thr, None, None, o, rgba, samples, error, C.byref(count), None, None)

    for call in (host, device):
        for base in (0, 1, 7):
            assert call(base=base) == -1
            assert b"halves" in L.rr_last_error() and b"equal" in L.rr_last_error() and str(base).encode() in L.rr_last_error()
        assert call(top=0) == -1                                  # rr_render's rule for a sample count
        assert b"samples" in L.rr_last_error()
        assert call(top=16383) == -2                              # ... and for the built-in table
        assert call(base=16384) == -2
        assert call(thr=float("nan")) == -1
        assert b"NaN" in L.rr_last_error()
        assert call(o=None) == -1
        assert b"out" in L.rr_last_error()
        assert call(scene=None) == -1
        assert call(camera=_camera(0, 38)) == -1                  # width == 0
        assert call(camera=_camera(32768, 16385)) == -2           # 2 x 2^29 + 65536 slots: refused before anything is allocated
        assert b"2^30" in L.rr_last_error()
        assert call(camera=_camera(65536, 2)) == -1               # a coordinate that does not fit 16 bits
    # the device form's alignment rules
    assert device(o=C.c_void_p(C.addressof(out) + 8)) == -1
    assert b"aligned" in L.rr_last_error()
    assert device(samples=C.c_void_p(C.addressof(out) + 1)) == -1
    assert b"aligned" in L.rr_last_error()
    assert device(error=C.c_void_p(C.addressof(out) + 2)) == -1 and device(rgba=C.c_void_p(C.addressof(out) + 2)) == -1

    # rr_refine_list_device
    lst = np.full(capi.refine_list_capacity(50, 38), 0x5a5a5a5a, np.uint32)
    lst_p = lst.ctypes.data_as(C.c_void_p)

    def refine(w=50, h=38, parts=out_p, thr=0.1, error=None, lp=lst_p, cnt=C.byref(count), scene=fake):
        return L.rr_refine_list_device(scene, w, h, parts, thr, error, lp, cnt, None)

    assert refine(w=0) == -1 and refine(h=0) == -1
    assert b"frame size" in L.rr_last_error()
    assert refine(w=65536, h=1) == -1
    assert refine(w=32768, h=16385) == -2
    assert b"2^30" in L.rr_last_error()
    assert refine(thr=float("nan")) == -1
    assert b"NaN" in L.rr_last_error()
    assert refine(parts=None) == -1 and refine(lp=None) == -1 and refine(cnt=None) == -1 and refine(scene=None) == -1
    assert refine(parts=C.c_void_p(C.addressof(out) + 8)) == -1
    assert b"parts_dev" in L.rr_last_error() and b"aligned" in L.rr_last_error()
    assert refine(lp=C.c_void_p(lst.ctypes.data + 2)) == -1 and refine(error=C.c_void_p(C.addressof(out) + 2)) == -1
    assert bytes(out) == b"\x5a" * C.sizeof(out) and (lst == 0x5a5a5a5a).all() and count.value == 77


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
    for n in NEW + ("rr_refine_list_capacity",):
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
        assert getattr(capi.lib(), n).argtypes is not None
    assert "rr_api_adaptive.h" in capi.LIB_SOURCES and "rr_adaptive.h" in capi.LIB_SOURCES
    for m in ("refine_list_device", "render_adaptive", "render_adaptive_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "render_adaptive_torch") and hasattr(renderer.Raytracing, "render_adaptive_on_device")
