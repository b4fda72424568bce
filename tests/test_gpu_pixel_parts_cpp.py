"""Raytracing::render_pixel_parts and render_pixel_parts_device of include/rustray_host.hpp, driven through host_shim.cpp: a list and the
whole frame give the records the ctypes binding gives, and the refusals of rr_render_pixel_parts come back through the C++ layer."""
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
    L.rh_render_pixel_parts.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rh_render_pixel_parts_device.argtypes = [C.c_void_p] + camera + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _equal(rec, prec, want, idx, K):
    p = want["parts"]
    assert np.array_equal(rec[:, 0:3], want["color"][idx].view(np.uint32)) and np.array_equal(rec[:, 3], want["depth"][idx].view(np.uint32))
    assert np.array_equal(rec[:, 4:7], want["normal"][idx].view(np.uint32)) and np.array_equal(rec[:, 7], want["object_id"][idx])
    prec = prec.reshape(len(idx), K, 8)
    assert np.array_equal(prec[:, :, 0:3], p["color"][idx].view(np.uint32)) and np.array_equal(prec[:, :, 3], p["depth"][idx].view(np.uint32))
    assert np.array_equal(prec[:, :, 4:7], p["normal"][idx].view(np.uint32)) and np.array_equal(prec[:, :, 7], p["object_id"][idx])


def test_render_pixel_parts_through_the_cpp_host_layer(hip, oracle):
    import torch
    fs = load_scene("monkey")                      # a mesh in front of nothing: hits, misses and NaN normals in one frame
    camera = camera_for(fs, W, H)
    cam = camera.c_struct()
    K = 4
    cfg = make_config(samples=8, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(fs, 0) as ds:             # (the C++ layer uses the library's built-in sub-sample table)
        want = ds.render_pixel_parts(cam, cfg, None, n_parts=K)
    assert np.isnan(want["parts"]["normal"]).any() and (want["parts"]["depth"] > 0).any()
    L = _shim()
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        idx = [3, 777, N - 1, 777, 1234]
        xy = np.array([(i % W) | ((i // W) << 16) for i in idx], np.uint32)
        rec, prec = np.zeros((5, 8), np.uint32), np.zeros((5 * K, 8), np.uint32)
        assert L.rh_render_pixel_parts(h, *args, xy.ctypes.data, 5, K, rec.ctypes.data, prec.ctypes.data) == 5
        _equal(rec, prec, want, idx, K)
        rec, prec = np.zeros((N, 8), np.uint32), np.zeros((N * K, 8), np.uint32)
        assert L.rh_render_pixel_parts(h, *args, None, 0, K, rec.ctypes.data, prec.ctypes.data) == N
        _equal(rec, prec, want, list(range(N)), K)
        # refused: a part count that is no power of two, one that does not divide the samples, an entry outside the frame
        for k in (3, 16):
            assert L.rh_render_pixel_parts(h, *args, xy.ctypes.data, 5, k, rec.ctypes.data, prec.ctypes.data) == -1
        assert L.rh_render_pixel_parts(h, *args, np.array([W], np.uint32).ctypes.data, 1, K, rec.ctypes.data, prec.ctypes.data) == -1
        # the device form
        txy = torch.from_numpy(xy.view(np.int32)).cuda()
        out = torch.zeros((N, 8), dtype=torch.int32, device="cuda")
        parts = torch.zeros((N * K, 8), dtype=torch.int32, device="cuda")

        def dev(xy_p, n, k, cancel=None):
            return L.rh_render_pixel_parts_device(h, *args, xy_p, n, k, out.data_ptr(), parts.data_ptr(), None, cancel)
        assert dev(txy.data_ptr(), 5, K) == 0
        torch.cuda.synchronize()
        _equal(out.cpu().numpy().view(np.uint32)[:5], parts.cpu().numpy().view(np.uint32)[:5 * K], want, idx, K)
        assert dev(txy.data_ptr(), 5, 1) == -1 and dev(txy.data_ptr(), 5, 16) == -1 and dev(None, N - 1, K) == -1
        flag = C.c_int(1)
        assert dev(txy.data_ptr(), 5, K, C.byref(flag)) == -6
        assert dev(None, N, K) == 0
        torch.cuda.synchronize()
        _equal(out.cpu().numpy().view(np.uint32), parts.cpu().numpy().view(np.uint32), want, list(range(N)), K)
    finally:
        L.rh_scene_destroy(h)
