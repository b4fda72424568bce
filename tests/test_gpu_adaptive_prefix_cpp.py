"""Raytracing::render_pixel_prefix, render_adaptive_prefix and render_adaptive_prefix_device of include/rustray_host.hpp, driven through
host_shim.cpp: the prefix and the frame refined on its prefixes equal what the ctypes binding gives, and a refusal comes back through
the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import camera_for, load_scene
from tests.test_cpp_host import _cam_args
from tests.test_gpu_adaptive_levels_cpp import H, N, W, _equal, _shim

pytestmark = pytest.mark.gpu

LADDER, THRESHOLD = (6, 14, 30), 0.1


def test_prefix_calls_through_the_cpp_host_layer(hip):
    import torch
    fs = load_scene("spheres_room")
    camera = camera_for(fs, W, H)
    cam = camera.c_struct()
    cfg = make_config(samples=30, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(fs, 0) as ds:             # (the C++ layer uses the library's built-in sub-sample tables)
        want = ds.render_adaptive_prefix(cam, cfg, LADDER, THRESHOLD, rgba8=True)
        want14 = ds.render_pixel_prefix(cam, cfg, None, samples_used=14, halves=True, rgba8=True)
    assert N > want["level_pixels"][1] > want["level_pixels"][2] > 0
    L = _shim()
    camera_t = L.rh_render_adaptive_levels.argtypes[1:10]
    L.rh_render_pixel_prefix.argtypes = [C.c_void_p] + camera_t + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_adaptive_prefix.argtypes = L.rh_render_adaptive_levels.argtypes
    L.rh_render_adaptive_prefix_device.argtypes = L.rh_render_adaptive_levels_device.argtypes
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    lv = (C.c_uint16 * 3)(*LADDER)
    short = (C.c_uint16 * 3)(6, 14, 28)
    try:
        # the prefix
        rec, hv, rgba = np.zeros((N, 8), np.uint32), np.zeros((N, 2, 8), np.uint32), np.zeros(4 * N, np.uint8)
        assert L.rh_render_pixel_prefix(h, *args, None, N, 14, rec.ctypes.data, hv.ctypes.data, rgba.ctypes.data) == N
        assert np.array_equal(rec[:, 0:3], want14["color"].view(np.uint32)) and np.array_equal(rec[:, 7], want14["object_id"])
        assert np.array_equal(hv[:, :, 0:3], want14["parts"]["color"].view(np.uint32)) and np.array_equal(rgba.reshape(N, 4), want14["rgba"])
        assert L.rh_render_pixel_prefix(h, *args, None, N, 13, rec.ctypes.data, hv.ctypes.data, None) == -1        # odd with halves
        assert L.rh_render_pixel_prefix(h, *args, None, N, 31, rec.ctypes.data, None, None) == -1                 # beyond the frame
        # the fused ladder
        rec, samples, error, rgba = np.zeros((N, 8), np.uint32), np.zeros(N, np.uint16), np.zeros(N, np.float32), np.zeros(4 * N, np.uint8)
        lp = np.full(4, 77, np.uint32)
        assert L.rh_render_adaptive_prefix(h, *args, lv, 3, THRESHOLD, rec.ctypes.data, samples.ctypes.data, error.ctypes.data, rgba.ctypes.data, lp.ctypes.data) == 0
        _equal(rec, samples, error, rgba, want)
        assert list(lp) == want["level_pixels"] + [77]
        rec2 = np.zeros((N, 8), np.uint32)
        assert L.rh_render_adaptive_prefix(h, *args, lv, 3, THRESHOLD, rec2.ctypes.data, None, None, None, None) == 0
        assert np.array_equal(rec2, rec)
        assert L.rh_render_adaptive_prefix(h, *args, short, 3, THRESHOLD, rec2.ctypes.data, None, None, None, None) == -1     # does not end at config.samples
        assert L.rh_render_adaptive_prefix(h, *args, lv, 1, THRESHOLD, rec2.ctypes.data, None, None, None, None) == -1
        # the device form
        out = torch.zeros((N, 8), dtype=torch.int32, device="cuda")
        t_rgba = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
        t_samples = torch.zeros((N,), dtype=torch.int16, device="cuda")
        t_error = torch.zeros((N,), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lp = np.full(4, 77, np.uint32)

        def dev(ladder, cancel=None):
            return L.rh_render_adaptive_prefix_device(h, *args, ladder, 3, THRESHOLD, out.data_ptr(), t_rgba.data_ptr(), t_samples.data_ptr(), t_error.data_ptr(),
                                                      lp.ctypes.data, None, cancel)
        assert dev(short) == -1
        flag = C.c_int(1)
        assert dev(lv, C.byref(flag)) == -6
        assert dev(lv) == 0 and list(lp) == want["level_pixels"] + [77]
        torch.cuda.synchronize()
        _equal(out.cpu().numpy().view(np.uint32), t_samples.cpu().numpy().view(np.uint16), t_error.cpu().numpy(), t_rgba.cpu().numpy(), want)
    finally:
        L.rh_scene_destroy(h)
