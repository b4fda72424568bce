"""Raytracing::accumulate_split and Raytracing::accumulate_split_device of include/rustray_host.hpp, driven through host_shim.cpp: the
layers the numpy yardstick gives, and a refusal of rr_accumulate_split_records coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config
from rustray_amd.temporal import accumulate_split_records
from tests.denoise_cases import F
from tests.helpers import load_scene
from tests.temporal_cases import frame_params
from tests.temporal_split_cases import split_frame_odd
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 37, 19
N = W * H
INPUTS = ("records", "halves", "diffuse", "diffuse_halves", "history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length", "motion")
OUTPUTS = (("records", (N, 8)), ("halves", (N, 2, 8)), ("diffuse", (N, 3)), ("diffuse_halves", (N, 2, 3)), ("length", (N,)))


def test_accumulate_split_through_the_cpp_host_layer(hip):
    import torch
    case = split_frame_odd(W, H)
    camera, prm = case["cam"], frame_params(case)
    want = accumulate_split_records(*(case[k] for k in INPUTS), camera, prm)
    first = accumulate_split_records(case["records"], None, case["diffuse"], None, None, None, None, None, None, None, camera, prm)
    fs = load_scene("spheres_room")
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_accumulate_split.argtypes = [C.c_void_p] + cam_types + [C.c_void_p] * 17 + [C.c_int, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda a: a.ctypes.data
    cprm = capi.accumulate_params(prm)
    try:
        out = {k: np.zeros(shape, F) for k, shape in OUTPUTS}
        # (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        assert L.rh_accumulate_split(h, *args, C.addressof(cprm), *(P(case[k]) for k in INPUTS), *(P(out[k]) for k, _ in OUTPUTS), None, 0, None) == 0
        for key, _ in OUTPUTS:
            assert np.array_equal(out[key].view(np.uint32), want[key].view(np.uint32)), key
        # the first frame, one layer, the library's default parameters
        assert L.rh_accumulate_split(h, *args, None, P(case["records"]), None, P(case["diffuse"]), None, None, None, None, None, None, None, P(out["records"]), None,
                                     P(out["diffuse"]), None, P(out["length"]), None, 0, None) == 0
        for key in ("records", "diffuse", "length"):
            assert np.array_equal(out[key].view(np.uint32), first[key].view(np.uint32)), key
        # the device form
        dev = {k: torch.from_numpy(np.ascontiguousarray(case[k]).copy()).cuda() for k in INPUTS}
        d_out = {k: torch.zeros(shape, device="cuda") for k, shape in OUTPUTS}
        torch.cuda.synchronize()
        assert L.rh_accumulate_split(h, *args, C.addressof(cprm), *(dev[k].data_ptr() for k in INPUTS), *(d_out[k].data_ptr() for k, _ in OUTPUTS), None, 1, None) == 0
        torch.cuda.synchronize()
        for key, _ in OUTPUTS:
            assert np.array_equal(d_out[key].cpu().numpy().view(np.uint32), want[key].view(np.uint32)), key
        # a refusal comes back through the layer
        assert L.rh_accumulate_split(h, *args, C.addressof(cprm), P(case["records"]), P(case["halves"]), P(case["diffuse"]), None, None, None, None, None, None, None,
                                     P(out["records"]), P(out["halves"]), P(out["diffuse"]), P(out["diffuse_halves"]), P(out["length"]), None, 0, None) == -1
        assert b"diffuse_halves is required" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
