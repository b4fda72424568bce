"""Raytracing::trace_shadow of include/rustray_host.hpp, driven through host_shim.cpp (rh_trace_shadow): a few dozen logged shadow
rays of the blocker scene, one call each, with no limit and at the light's distance, against the oracle's log."""
import ctypes as C
import os

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import rr_flat_scene
from tests import shadow_ray_cases as cases

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_trace_shadow_through_the_cpp_host_layer(hip, oracle):
    fs, rays = cases.corner_case(oracle, "blocker")
    idx = np.concatenate([np.flatnonzero(rays["found"])[:24], np.flatnonzero(~rays["found"])[:24]])
    sub = cases.subset(rays, idx)
    assert sub["found"].sum() == 24 and (sub["depth"] == 1).all()
    L = C.CDLL(SHIM)
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_trace_shadow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        o = np.ascontiguousarray(sub["origin"], np.float32); d = np.ascontiguousarray(sub["dir"], np.float32)
        n_occ = {}
        for cname in ("none", "light0", "t", "below_t"):
            lim = cases.limit_classes(fs, sub)[cname]
            out = np.zeros((len(idx), 4), np.uint32)
            assert L.rh_trace_shadow(h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                     None if lim is None else lim.ctypes.data_as(C.c_void_p), len(idx), 1, out.ctypes.data_as(C.c_void_p)) == 0
            got = (out[:, 0].astype(bool), out[:, 1].astype(np.int32), out[:, 2].copy(), out[:, 3].copy().view(np.float32))
            bad = cases.mismatches(got, sub, lim)
            assert len(bad) == 0, cases.describe(f"blocker / {cname}", sub, lim, bad, got)
            n_occ[cname] = int(got[0].sum())
        assert n_occ == {"none": 24, "light0": 0, "t": 24, "below_t": 0}
    finally:
        L.rh_scene_destroy(h)
