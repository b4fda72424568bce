"""Raytracing::accumulate_clamped_split and Raytracing::accumulate_clamped_split_device of include/rustray_host.hpp, driven through
host_shim.cpp: the layers the numpy yardstick gives, and a refusal of rr_accumulate_clamped_split_records coming back through the C++
layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config
from rustray_amd.temporal import HistoryClampParams, accumulate_clamped_split_records
from tests.denoise_cases import F, differing_words
from tests.helpers import load_scene
from tests.temporal_cases import frame_params
from tests.temporal_clamp_split_cases import KEYS, clamp_split_frame_odd, inputs
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 37, 19
N = W * H
OUTPUTS = (("records", (N, 8)), ("halves", (N, 2, 8)), ("diffuse", (N, 3)), ("diffuse_halves", (N, 2, 3)), ("length", (N,)))


def test_accumulate_clamped_split_through_the_cpp_host_layer(hip):
    import torch
    case = clamp_split_frame_odd(W, H)
    camera, prm = case["cam"], frame_params(case)
    a = dict(zip(KEYS, inputs(case, True, True, False)))
    want = accumulate_clamped_split_records(*a.values(), camera, prm, HistoryClampParams(2, 1.5))
    first = accumulate_clamped_split_records(case["records"], None, case["diffuse"], None, None, None, None, None, None, None, camera, prm)
    fs = load_scene("spheres_room")
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_accumulate_clamped_split.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 16 + [C.c_int, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda x: x.ctypes.data
    cprm = capi.accumulate_params(prm)

    def same(got, ref, what):
        for key, _ in OUTPUTS:
            if ref[key] is None:
                continue
            if key in ("diffuse", "diffuse_halves"):
                assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(ref[key]).view(np.uint32)), (what, key)
            else:
                assert differing_words(got[key], ref[key])[0] == 0, (what, key)
    try:
        out = {k: np.zeros(shape, F) for k, shape in OUTPUTS}
        # (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        assert L.rh_accumulate_clamped_split(h, *args, C.addressof(cprm), 2, 1.5, *(P(a[k]) for k in KEYS), *(P(out[k]) for k, _ in OUTPUTS), None, 0, None) == 0
        same(out, want, "host form")
        # the first frame, one layer, the library's default parameters and default clamp
        assert L.rh_accumulate_clamped_split(h, *args, None, 0, 0.0, P(case["records"]), None, P(case["diffuse"]), None, None, None, None, None, None, None,
                                             P(out["records"]), None, P(out["diffuse"]), None, P(out["length"]), None, 0, None) == 0
        same(dict(out, halves=None, diffuse_halves=None), first, "first frame")
        # the device form
        dev = {k: torch.from_numpy(np.ascontiguousarray(a[k]).copy()).cuda() for k in KEYS}
        d_out = {k: torch.zeros(shape, device="cuda") for k, shape in OUTPUTS}
        torch.cuda.synchronize()
        assert L.rh_accumulate_clamped_split(h, *args, C.addressof(cprm), 2, 1.5, *(dev[k].data_ptr() for k in KEYS), *(d_out[k].data_ptr() for k, _ in OUTPUTS),
                                             None, 1, None) == 0
        torch.cuda.synchronize()
        same({k: v.cpu().numpy() for k, v in d_out.items()}, want, "device form")
        # a refusal comes back through the layer: diffuse_out on diffuse
        ptrs = {k: dev[k].data_ptr() for k in KEYS}
        outs = {k: d_out[k].data_ptr() for k, _ in OUTPUTS}
        assert L.rh_accumulate_clamped_split(h, *args, C.addressof(cprm), 1, 1.0, *(ptrs[k] for k in KEYS),
                                             *(outs[k] if k != "diffuse" else ptrs["diffuse"] for k, _ in OUTPUTS), None, 1, None) == -1
        assert b"diffuse_out overlaps diffuse " in hip.lib().rr_last_error() and b"rr_accumulate_clamped_split_records_device" in hip.lib().rr_last_error()
        assert L.rh_accumulate_clamped_split(h, *args, C.addressof(cprm), 3, 1.0, *(P(a[k]) for k in KEYS), *(P(out[k]) for k, _ in OUTPUTS), None, 0, None) == -1
        assert b"clamp->radius" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
