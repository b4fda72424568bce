"""Raytracing::render_adaptive_levels and render_adaptive_levels_device of include/rustray_host.hpp, driven through host_shim.cpp: the frame
refined level by level equals what the ctypes binding gives, and a refusal of rr_render_adaptive_levels comes back through the C++ layer."""
import ctypes as C
import os

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_config, rr_flat_scene
from tests.helpers import camera_for, load_scene
from tests.test_cpp_host import _cam_args

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")
W, H = 50, 38
N = W * H
LEVELS, THRESHOLD = (6, 14, 30), 0.1


def _shim():
    assert os.path.exists(SHIM), f"{SHIM} is missing: run `make -C rustray_amd/csrc`"
    L = C.CDLL(SHIM)
    F3 = C.c_float * 3
    camera = [C.c_float, F3, F3, F3, C.c_float, C.c_float, C.POINTER(rr_config), C.c_uint32, C.c_uint32]
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_render_adaptive_levels.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_adaptive_levels_device.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                         C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _equal(rec, samples, error, rgba, want):
    assert np.array_equal(rec[:, 0:3], want["color"].view(np.uint32)) and np.array_equal(rec[:, 3], want["depth"].view(np.uint32))
    assert np.array_equal(rec[:, 4:7], want["normal"].view(np.uint32)) and np.array_equal(rec[:, 7], want["object_id"])
    assert np.array_equal(samples.astype(np.uint32), want["samples"]) and np.array_equal(error.view(np.uint32), want["error"].view(np.uint32))
    assert np.array_equal(rgba.reshape(N, 4), want["rgba"])


def test_render_adaptive_levels_through_the_cpp_host_layer(hip):
    import torch
    fs = load_scene("spheres_room")
    camera = camera_for(fs, W, H)
    cam = camera.c_struct()
    cfg = make_config(samples=6, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(fs, 0) as ds:             # (the C++ layer uses the library's built-in sub-sample tables)
        want = ds.render_adaptive_levels(cam, cfg, LEVELS, THRESHOLD, rgba8=True)
    assert N > want["level_pixels"][1] > want["level_pixels"][2] > 0
    L = _shim()
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    lv = (C.c_uint16 * 3)(*LEVELS)
    odd = (C.c_uint16 * 3)(6, 15, 30)
    try:
        rec, samples, error, rgba = np.zeros((N, 8), np.uint32), np.zeros(N, np.uint16), np.zeros(N, np.float32), np.zeros(4 * N, np.uint8)
        lp = np.full(4, 77, np.uint32)
        assert L.rh_render_adaptive_levels(h, *args, lv, 3, THRESHOLD, rec.ctypes.data, samples.ctypes.data, error.ctypes.data, rgba.ctypes.data, lp.ctypes.data) == 0
        _equal(rec, samples, error, rgba, want)
        assert list(lp) == want["level_pixels"] + [77]
        rec2 = np.zeros((N, 8), np.uint32)
        assert L.rh_render_adaptive_levels(h, *args, lv, 3, THRESHOLD, rec2.ctypes.data, None, None, None, None) == 0
        assert np.array_equal(rec2, rec)
        assert L.rh_render_adaptive_levels(h, *args, odd, 3, THRESHOLD, rec2.ctypes.data, None, None, None, None) == -1      # an odd count
        assert L.rh_render_adaptive_levels(h, *args, lv, 1, THRESHOLD, rec2.ctypes.data, None, None, None, None) == -1       # one level
        assert L.rh_render_adaptive_levels(h, *args, lv, 3, float("nan"), rec2.ctypes.data, None, None, None, None) == -1
        # the device form
        out = torch.zeros((N, 8), dtype=torch.int32, device="cuda")
        t_rgba = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
        t_samples = torch.zeros((N,), dtype=torch.int16, device="cuda")
        t_error = torch.zeros((N,), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lp = np.full(4, 77, np.uint32)

        def dev(levels, cancel=None):
            return L.rh_render_adaptive_levels_device(h, *args, levels, 3, THRESHOLD, out.data_ptr(), t_rgba.data_ptr(), t_samples.data_ptr(), t_error.data_ptr(),
                                                      lp.ctypes.data, None, cancel)
        assert dev(odd) == -1
        flag = C.c_int(1)
        assert dev(lv, C.byref(flag)) == -6
        assert dev(lv) == 0 and list(lp) == want["level_pixels"] + [77]
        torch.cuda.synchronize()
        _equal(out.cpu().numpy().view(np.uint32), t_samples.cpu().numpy().view(np.uint16), t_error.cpu().numpy(), t_rgba.cpu().numpy(), want)
    finally:
        L.rh_scene_destroy(h)
