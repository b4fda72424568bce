"""Raytracing::render(x, y), render_pixels and render_pixels_device of include/rustray_host.hpp, driven through host_shim.cpp: the
reference's own per-pixel signature gives the frame's PixelData, a list and the whole frame give the records the ctypes binding gives,
and the argument errors of rr_render_pixels come back through the C++ layer as they are."""
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


def _shim():
    assert os.path.exists(SHIM), f"{SHIM} is missing: run `make -C rustray_amd/csrc`"
    L = C.CDLL(SHIM)
    F3 = C.c_float * 3
    camera = [C.c_float, F3, F3, F3, C.c_float, C.c_float, C.POINTER(rr_config), C.c_uint32, C.c_uint32]
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_render_pixels.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rh_render_pixel.argtypes = [C.c_void_p] + camera + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.rh_render_pixels_device.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_pixels_from_on_pass.argtypes = [C.c_void_p] + camera + [C.c_void_p]
    return L


def test_render_pixels_through_the_cpp_host_layer(hip, oracle):
    import torch
    fs = load_scene("monkey")                      # a mesh in front of nothing: hits, misses and NaN normals in one frame
    camera = camera_for(fs, W, H)
    cam = camera.c_struct()
    cfg = make_config(samples=3, monte_carlo=True, seed=3, max_recursion=4, gamma_correction=True)
    with hip.DeviceScene(fs, 0) as ds:             # (the C++ layer uses the library's built-in sub-sample table)
        frame = ds.render(cam, cfg, aux=True)
        full = ds.render_pixels(cam, cfg, None, rgba8=True)
    depth = frame["depth"].reshape(N)
    hit, miss = int(np.flatnonzero(depth > 0)[0]), int(np.flatnonzero(depth == 0)[0])
    assert frame["object_id"].reshape(N)[hit] != 0 and np.isnan(frame["normal"].reshape(N, 3)[miss]).all()
    L = _shim()
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        # Raytracing::render(x, y): a hit, a miss and the last pixel of the frame
        for i in (hit, miss, N - 1):
            x, y = i % W, i // W
            out6, nd4 = np.zeros(6, np.int32), np.zeros(4, np.float32)
            assert L.rh_render_pixel(h, *args, x, y, out6.ctypes.data, nd4.ctypes.data) == 0
            assert out6[:3].tolist() == frame["rgba"].reshape(N, 4)[i, :3].tolist(), (x, y)
            assert int(out6[3]) == int(frame["object_id"].reshape(N)[i]) and (int(out6[4]), int(out6[5])) == (x, y)
            assert np.array_equal(nd4[:3], frame["normal"].reshape(N, 3)[i], equal_nan=True) and nd4[3] == depth[i]
        out6, nd4 = np.zeros(6, np.int32), np.zeros(4, np.float32)
        for x, y in ((W, 0), (0, H), (-1, 3)):
            assert L.rh_render_pixel(h, *args, x, y, out6.ctypes.data, nd4.ctypes.data) == -1 and out6[4] == -1
        # a list, and the whole frame
        xy = np.array([(i % W) | ((i // W) << 16) for i in (hit, miss, N - 1, hit, 777)], np.uint32)
        rec, rgba = np.zeros((5, 8), np.uint32), np.zeros((5, 4), np.uint8)
        assert L.rh_render_pixels(h, *args, xy.ctypes.data, 5, rec.ctypes.data, rgba.ctypes.data) == 5
        idx = [hit, miss, N - 1, hit, 777]
        assert np.array_equal(rec[:, 0:3], full["color"][idx].view(np.uint32)) and np.array_equal(rec[:, 3], full["depth"][idx].view(np.uint32))
        assert np.array_equal(rec[:, 4:7], full["normal"][idx].view(np.uint32)) and np.array_equal(rec[:, 7], full["object_id"][idx])
        assert np.array_equal(rgba, full["rgba"][idx]) and np.array_equal(rgba, frame["rgba"].reshape(N, 4)[idx])
        rec, rgba = np.zeros((N, 8), np.uint32), np.zeros((N, 4), np.uint8)
        assert L.rh_render_pixels(h, *args, None, 0, rec.ctypes.data, rgba.ctypes.data) == N
        assert np.array_equal(rec[:, 0:3], full["color"].view(np.uint32)) and np.array_equal(rgba, frame["rgba"].reshape(N, 4))
        assert L.rh_render_pixels(h, *args, np.array([W], np.uint32).ctypes.data, 1, rec.ctypes.data, None) == -1   # outside the frame
        # render_pixels_device, and the argument errors of the C ABI through it
        txy = torch.from_numpy(xy.view(np.int32)).cuda()
        out = torch.zeros((N, 8), dtype=torch.int32, device="cuda")

        def dev(cfg_, xy_p, n, cancel=None):
            a = _cam_args(camera) + (C.byref(cfg_), W, H)
            return L.rh_render_pixels_device(h, *a, xy_p, n, out.data_ptr(), None, None, cancel)
        assert dev(cfg, txy.data_ptr(), 5) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:5, 0:3], full["color"][idx].view(np.uint32))
        assert dev(cfg, None, N - 1) == -1                                           # no list: the whole frame or nothing
        assert dev(make_config(samples=0), txy.data_ptr(), 5) == -1
        assert dev(make_config(samples=16383), txy.data_ptr(), 5) == -2            # beyond the built-in table
        assert dev(make_config(samples=3, max_recursion=31), txy.data_ptr(), 5) == -2
        flag = C.c_int(1)
        assert dev(cfg, txy.data_ptr(), 5, C.byref(flag)) == -6
        assert dev(cfg, None, N) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:, 0:3], full["color"].view(np.uint32))
        # from on_pass of a progressive frame of the same scene: refused
        seen = np.zeros(2, np.uint32)
        a4 = _cam_args(camera) + (C.byref(make_config(samples=4, seed=1)), W, H)
        assert L.rh_render_pixels_from_on_pass(h, *a4, seen.ctypes.data) == 0
        assert seen[0] >= 1 and seen[1] == seen[0]
    finally:
        L.rh_scene_destroy(h)
