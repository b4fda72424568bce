"""Raytracing::accumulate_clamped and Raytracing::accumulate_clamped_device of include/rustray_host.hpp, driven through host_shim.cpp: the
layers the numpy yardstick gives, and a refusal of rr_accumulate_clamped_records coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config
from rustray_amd.temporal import HistoryClampParams, accumulate_clamped_records
from tests.denoise_cases import F, differing_words
from tests.helpers import load_scene
from tests.temporal_cases import frame_params
from tests.temporal_clamp_cases import KEYS, clamp_frame_odd
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 37, 19
N = W * H
OUTPUTS = (("records", (N, 8)), ("halves", (N, 2, 8)), ("length", (N,)))


def test_accumulate_clamped_through_the_cpp_host_layer(hip):
    import torch
    case = clamp_frame_odd(W, H)
    camera, prm = case["cam"], frame_params(case)
    want = accumulate_clamped_records(*(case[k] for k in KEYS), camera, prm, HistoryClampParams(2, 1.5))
    first = accumulate_clamped_records(case["records"], None, None, None, None, None, camera, prm)
    fs = load_scene("spheres_room")
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_accumulate_clamped.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda a: a.ctypes.data
    cprm = capi.accumulate_params(prm)

    def same(got, ref, what):
        for key, _ in OUTPUTS:
            if ref[key] is not None:
                assert differing_words(got[key], ref[key])[0] == 0, (what, key)
    try:
        out = {k: np.zeros(shape, F) for k, shape in OUTPUTS}
        # (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        assert L.rh_accumulate_clamped(h, *args, C.addressof(cprm), 2, 1.5, *(P(case[k]) for k in KEYS), *(P(out[k]) for k, _ in OUTPUTS), None, 0, None) == 0
        same(out, want, "host form")
        # the first frame, one layer, the library's default parameters and default clamp
        assert L.rh_accumulate_clamped(h, *args, None, 0, 0.0, P(case["records"]), None, None, None, None, None, P(out["records"]), None, P(out["length"]), None, 0, None) == 0
        same(dict(out, halves=None), first, "first frame")
        # the device form
        dev = {k: torch.from_numpy(np.ascontiguousarray(case[k]).copy()).cuda() for k in KEYS}
        d_out = {k: torch.zeros(shape, device="cuda") for k, shape in OUTPUTS}
        torch.cuda.synchronize()
        assert L.rh_accumulate_clamped(h, *args, C.addressof(cprm), 2, 1.5, *(dev[k].data_ptr() for k in KEYS), *(d_out[k].data_ptr() for k, _ in OUTPUTS), None, 1, None) == 0
        torch.cuda.synchronize()
        same({k: v.cpu().numpy() for k, v in d_out.items()}, want, "device form")
        # a refusal comes back through the layer: out on records
        assert L.rh_accumulate_clamped(h, *args, C.addressof(cprm), 1, 1.0, dev["records"].data_ptr(), None, None, None, None, None, dev["records"].data_ptr(), None,
                                       d_out["length"].data_ptr(), None, 1, None) == -1
        assert b"out overlaps records" in hip.lib().rr_last_error()
        assert L.rh_accumulate_clamped(h, *args, C.addressof(cprm), 3, 1.0, *(P(case[k]) for k in KEYS), *(P(out[k]) for k, _ in OUTPUTS), None, 0, None) == -1
        assert b"clamp->radius" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
