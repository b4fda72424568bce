"""Raytracing::trace_device / trace_shadow_device / shade_device of include/rustray_host.hpp, driven through host_shim.cpp
(rh_trace_device, rh_trace_shadow_device, rh_shade_device): one closest-hit, one shadow and one radiance call of 257 rays on
device buffers give the bytes of the Python path (capi.DeviceScene on a handle of its own)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rustray_amd import capi
from rustray_amd.flat import rr_config, rr_flat_scene
from tests.test_gpu_ray_queries_device import (_dev, _light_distances, _rays, _scene, _sentinel, _shade_cfg, dev_shade, dev_shadow, dev_trace)

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_device_queries_through_the_cpp_host_layer(hip, oracle):
    n = 257
    fs = _scene("packet_40")
    o, d = (a[:n] for a in _rays(oracle, shadow=True))
    lim = _light_distances(fs, o)
    cfg = _shade_cfg()
    ids = (np.arange(n, dtype=np.uint32) * np.uint32(5) + np.uint32(1)).astype(np.uint32)
    with hip.DeviceScene(fs, 0) as ds:
        want = dict(closest=dev_trace(ds, o, d, 2), shadow=dev_shadow(ds, o, d, lim, 2), shade=dev_shade(ds, cfg, o, d, n, 1, ids))
    L = C.CDLL(SHIM)
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_trace_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rh_trace_shadow_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rh_shade_device.argtypes = [C.c_void_p, C.POINTER(rr_config), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        to, td, tl, ti = _dev(o), _dev(d), _dev(lim), _dev(ids.view(np.int32))
        out = dict(closest=_sentinel(n, 5), shadow=_sentinel(n, 5), shade=_sentinel(n, 8))
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        sp = C.c_void_p(st.cuda_stream)
        assert L.rh_trace_device(h, to.data_ptr(), td.data_ptr(), n, 2, out["closest"].data_ptr(), sp) == 0
        assert L.rh_trace_shadow_device(h, to.data_ptr(), td.data_ptr(), tl.data_ptr(), n, 2, out["shadow"].data_ptr(), sp) == 0
        assert L.rh_shade_device(h, C.byref(cfg), to.data_ptr(), td.data_ptr(), n, 1, ti.data_ptr(), out["shade"].data_ptr(), sp) == 0
        st.synchronize()
        for k, t in out.items():
            got = t.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want[k]), f"{k}: {int((got != want[k]).any(axis=1).sum())} of {n} records differ"
        assert (want["closest"][:, 0] == 1).any() and (want["shadow"][:, 0] == 1).any() and (want["shadow"][:, 0] == 0).any()
        # a refusal comes back as the status code
        assert L.rh_trace_device(h, to.data_ptr(), td.data_ptr(), n, 0, out["closest"].data_ptr(), sp) == -1
    finally:
        L.rh_scene_destroy(h)
