"""Raytracing::surface / surface_device of include/rustray_host.hpp, driven through host_shim.cpp (rh_surface_rays,
rh_surface_rays_device): the 1 900 rays of tests/test_gpu_surface_rays.py on the 20-item textured scene give, from host arrays and
from device buffers, the bytes of the C ABI's answer (capi.DeviceScene on a handle of its own)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rustray_amd import capi
from rustray_amd.flat import rr_flat_scene
from tests.test_gpu_surface_rays import N, SENTINEL, _bytes, _case

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_surface_queries_through_the_cpp_host_layer(hip, oracle):
    c = _case(hip, oracle, "rich")
    o, d, want = c["o"], c["d"], _bytes(c["got"])
    L = C.CDLL(SHIM)
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_surface_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rh_surface_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    cs = c["fs"].c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        out = np.full((N, 32), SENTINEL, np.uint32)
        assert L.rh_surface_rays(h, o.ctypes.data, d.ctypes.data, N, 1, out.ctypes.data) == 0
        assert np.array_equal(_bytes(out), want), f"{int((_bytes(out) != want).any(axis=1).sum())} of {N} records differ"
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        dev = torch.full((N, 32), SENTINEL, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert L.rh_surface_rays_device(h, to.data_ptr(), td.data_ptr(), N, 1, dev.data_ptr(), C.c_void_p(st.cuda_stream)) == 0
        st.synchronize()
        got = _bytes(dev.cpu().numpy())
        assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} of {N} records differ"
        assert (c["got"]["hit"] == 1).any() and (c["got"]["hit"] == 0).any()
        # a refusal comes back as the status code (device form) or as no records (host form)
        assert L.rh_surface_rays_device(h, to.data_ptr(), td.data_ptr(), N, 0, dev.data_ptr(), C.c_void_p(st.cuda_stream)) == -1
        assert L.rh_surface_rays(h, o.ctypes.data, d.ctypes.data, N, 0, out.ctypes.data) == -1
    finally:
        L.rh_scene_destroy(h)
