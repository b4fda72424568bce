"""Raytracing::denoise and Raytracing::render_denoised of include/rustray_host.hpp, driven through host_shim.cpp: the records the numpy
yardstick gives, and a refusal of rr_denoise_records coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi, denoise
from rustray_amd.denoise import DenoiseParams, atrous_denoise
from rustray_amd.flat import make_config
from rustray_amd.renderer import _pack_records
from tests.denoise_cases import F, random_frame
from tests.helpers import camera_for, load_scene
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H


def test_denoise_through_the_cpp_host_layer(hip):
    fs = load_scene("spheres_room")
    camera = camera_for(fs, W, H)
    cfg = make_config(samples=8, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(fs, 0) as ds:             # (the C++ layer uses the library's built-in sub-sample table)
        base = ds.render_pixel_parts(camera.c_struct(), cfg, None, n_parts=2)
    noisy_want = _pack_records(base)
    want = atrous_denoise(noisy_want, _pack_records(base["parts"]), None, W, H)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_denoise.argtypes = [C.c_void_p] + cam_types + [C.c_void_p] * 7
    L.rh_render_denoised.argtypes = [C.c_void_p] + cam_types + [C.c_void_p] * 4
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        out, noisy, rgba = np.zeros((N, 8), F), np.zeros((N, 8), F), np.zeros((N, 4), np.uint8)
        assert L.rh_render_denoised(h, *args, None, out.ctypes.data, rgba.ctypes.data, noisy.ctypes.data) == 0
        assert np.array_equal(noisy.view(np.uint32), noisy_want.view(np.uint32))
        assert np.array_equal(out.view(np.uint32), want["records"].view(np.uint32))
        assert np.array_equal(rgba, denoise.frame_bytes_linear(want["records"][:, 0:3]))
        # hand-made records with an albedo and parameters of the caller's
        records, halves, albedo = random_frame(W, H)
        prm = DenoiseParams(iterations=4, normal_power_log2=2, sigma_depth=0.2, sigma_luminance=3.0)
        want2 = atrous_denoise(records, halves, albedo, W, H, prm)
        cprm = capi.denoise_params(prm)
        var = np.zeros(N, F)
        assert L.rh_denoise(h, *args, records.ctypes.data, halves.ctypes.data, albedo.ctypes.data, C.addressof(cprm), out.ctypes.data, var.ctypes.data, None) == 0
        assert np.array_equal(out.view(np.uint32), want2["records"].view(np.uint32)) and np.array_equal(var.view(np.uint32), want2["variance"].view(np.uint32))
        cprm.iterations = 7
        assert L.rh_denoise(h, *args, records.ctypes.data, None, None, C.addressof(cprm), out.ctypes.data, None, None) == -1
        assert b"iterations" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
