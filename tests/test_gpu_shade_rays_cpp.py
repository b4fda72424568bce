"""Raytracing::shade_rays of include/rustray_host.hpp, driven through host_shim.cpp (rh_shade_rays): 48 rays of the spheres_room
frame (16 results of 3) with the handle's config must give the records the ctypes binding gives."""
import ctypes as C
import os

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import rr_config, rr_flat_scene
from tests.test_gpu_shade_rays import S, _case

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_shade_rays_through_the_cpp_host_layer(hip, oracle):
    c = _case(hip, oracle, "spheres_room", need_ref=False)
    first = 700                                    # results 700 .. 715 of the frame: a row of pixels across the room
    o = np.ascontiguousarray(c["o"][first * S:(first + 16) * S]); d = np.ascontiguousarray(c["d"][first * S:(first + 16) * S])
    ids = np.arange(first, first + 16, dtype=np.uint32)
    assert len(o) == 48
    L = C.CDLL(SHIM)
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_shade_rays.argtypes = [C.c_void_p, C.POINTER(rr_config), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    cs = c["fs"].c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        out = np.zeros((16, 8), np.uint32)
        assert L.rh_shade_rays(h, C.byref(c["cfg"]), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), 48, S,
                               ids.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        lone = np.zeros((48, 8), np.uint32)        # one record per ray, ids = the ray's index
        assert L.rh_shade_rays(h, C.byref(c["cfg"]), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), 48, 1, None, lone.ctypes.data_as(C.c_void_p)) == 0
        assert L.rh_shade_rays(h, C.byref(c["cfg"]), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), 47, S, None, out.ctypes.data_as(C.c_void_p)) == -1
    finally:
        L.rh_scene_destroy(h)
    want = c["got"]
    sel = slice(first, first + 16)
    assert np.array_equal(out[:, 0:3], want["color"][sel].view(np.uint32))
    assert np.array_equal(out[:, 3], want["depth"][sel].view(np.uint32))
    assert np.array_equal(out[:, 4:7], want["normal"][sel].view(np.uint32))
    assert np.array_equal(out[:, 7], want["object_id"][sel]) and (out[:, 7] != 0).all()
    with hip.DeviceScene(c["fs"], 0) as ds:
        single = ds.shade_rays(o, d, c["cfg"], 1)
    assert np.array_equal(lone[:, 0:3], single["color"].view(np.uint32)) and np.array_equal(lone[:, 7], single["object_id"])
