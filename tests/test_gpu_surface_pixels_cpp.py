"""Raytracing::surface_pixels, ::albedo and ::surface_pixels_device of include/rustray_host.hpp, driven through host_shim.cpp: the bytes the
Python layer gives for the same scene and camera, and a refusal of rr_surface_pixels coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import SURFACE_HIT_DTYPE, make_config
from tests.helpers import camera_for
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H


def test_surface_pixels_through_the_cpp_host_layer(hip):
    import torch
    from tools.fuzz_parity import rich_scene
    fs = rich_scene(9119)
    camera = camera_for(fs, W, H)
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    rng = np.random.default_rng(5)
    xy = (rng.integers(0, W, 65) | (rng.integers(0, H, 65) << 16)).astype(np.uint32)
    at = (xy >> 16) * W + (xy & 0xffff)
    with hip.DeviceScene(fs, 0) as ds:
        want, want_albedo = ds.surface_pixels(camera.c_struct())
    assert (want["hit"] == 1).any() and (want["hit"] == 0).any()
    bytes_of = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_surface_pixels.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rh_surface_pixels_device.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda a: a.ctypes.data
    try:
        # the whole frame, records and albedo (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        rec, albedo = np.zeros(N, SURFACE_HIT_DTYPE), np.ones((N, 3), np.float32)
        assert L.rh_surface_pixels(h, *args, None, 0, P(rec), P(albedo)) == 0
        assert np.array_equal(bytes_of(rec), bytes_of(want)) and np.array_equal(albedo.view(np.uint32), want_albedo.view(np.uint32))
        # a list, records alone
        listed = np.zeros(65, SURFACE_HIT_DTYPE)
        assert L.rh_surface_pixels(h, *args, P(xy), 65, P(listed), None) == 0
        assert np.array_equal(bytes_of(listed), bytes_of(want[at]))
        # the device form: the whole frame's albedo alone, then a list with both
        d_albedo = torch.ones((N, 3), device="cuda")
        assert L.rh_surface_pixels_device(h, *args, None, N, None, d_albedo.data_ptr(), None) == 0
        d_xy = torch.from_numpy(xy.view(np.int32)).cuda()
        d_rec, d_alb = torch.zeros((65, 32), device="cuda"), torch.ones((65, 3), device="cuda")
        assert L.rh_surface_pixels_device(h, *args, d_xy.data_ptr(), 65, d_rec.data_ptr(), d_alb.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_albedo.cpu().numpy().view(np.uint32), want_albedo.view(np.uint32))
        assert np.array_equal(d_rec.cpu().numpy().view(np.uint8).reshape(65, 128), bytes_of(want[at]))
        assert np.array_equal(d_alb.cpu().numpy().view(np.uint32), want_albedo[at].view(np.uint32))
        # refusals come back through the layer
        bad = xy.copy()
        bad[7] = W | (3 << 16)
        assert L.rh_surface_pixels(h, *args, P(bad), 65, P(listed), None) == -1
        assert b"pixel_xy[7] = (50, 3)" in hip.lib().rr_last_error()
        assert L.rh_surface_pixels_device(h, *args, None, N, None, None, None) == -1 and b"both NULL" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
